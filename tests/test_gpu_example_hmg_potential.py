"""GPU test of examples/hmg_potential.cpp (the C ABI alone): the RF potential problem at p = 2 on a Cartesian mesh
refined twice, solved with Jacobi-PCG, with the PCG preconditioned by the p-only V-cycle 1 -> 2 on the finest mesh
and with the PCG preconditioned by the V-cycle (h0, 1) -> (h1, 1) -> (h2, 1) -> (h2, 2) -- exit status 0 (all
converged, the solutions agree, the manufactured solution is met, h+p V-cycle < p V-cycle < Jacobi in iterations)
and the three iteration counts printed."""
import os
import re
import subprocess

import pytest

import helpers

pytestmark = pytest.mark.gpu


def test_example_hmg_potential_on_gpu():
    examples = os.path.join(helpers.ROOT, "examples")
    binary = os.path.join(examples, "hmg_potential")
    if not os.access(binary, os.X_OK):
        subprocess.run(["make", "-s", "-C", examples], check=True, timeout=300)
    r = subprocess.run([binary], cwd=helpers.ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = [re.search(rf"^{k}-PCG iterations: (\d+)", r.stdout, re.M) for k in ("Jacobi", "p V-cycle", r"h\+p V-cycle")]
    assert all(counts)
    jac, pmg, hpmg = (int(c.group(1)) for c in counts)
    assert 0 < hpmg < pmg < jac
    assert r.stdout.rstrip().endswith("PASS")
