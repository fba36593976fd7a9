"""GPU test of examples/rf_electrode.cpp (the C ABI alone): the electrode problem with inhomogeneous essential data on
two boundary attributes -- the marked essential list, the device elimination, the PCG from the lifted data -- and its
Joule power: exit status 0 (converged, the data kept bitwise, the closed-form potential and power met to the CPU
oracle's own discretisation values plus 25 %, the power equal to the energy, the sigma = 1 potential exact) and a
final PASS."""
import os
import re
import subprocess

import pytest

import helpers

pytestmark = pytest.mark.gpu


def test_example_rf_electrode_on_gpu():
    examples = os.path.join(helpers.ROOT, "examples")
    binary = os.path.join(examples, "rf_electrode")
    if not os.access(binary, os.X_OK):
        subprocess.run(["make", "-s", "-C", examples], check=True, timeout=300)
    r = subprocess.run([binary], cwd=helpers.ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    it = re.search(r"Jacobi-PCG from the lifted data: (\d+) iterations \(converged 1\), essential data kept bitwise 1",
                   r.stdout)
    assert it and int(it.group(1)) > 0
    assert r.stdout.rstrip().endswith("PASS")
