"""examples/rf_heat_step.cpp: a native caller of the linear form and the sourced ODE step through
include/ecm2_pa.h alone -- the Joule heat of a linear potential on the unit cube and one SDIRK33
step from a uniform temperature, checked against their closed forms (sum b = sigma |a|^2,
u1 = u0 + dt sigma |a|^2 / rho c)."""
import os
import subprocess

import pytest

from helpers import ROOT

EXAMPLES = os.path.join(ROOT, "examples")
BINARY = os.path.join(EXAMPLES, "rf_heat_step")


def _build():
    subprocess.run(["make", "-s", "-C", EXAMPLES], check=True, timeout=300)
    assert os.access(BINARY, os.X_OK)


def test_rf_example_builds_and_fails_loudly_without_gpu():
    """Compiles and links against the header + library; with no device the linear form's create
    returns ECM2_ERR_HIP and the program stops (no CPU fallback)."""
    _build()
    import ecm2_amd as E
    if E.load_library().ecm2_device_count() > 0:
        pytest.skip("a GPU is visible")
    r = subprocess.run([BINARY], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "unit cube 4^3 elements" in r.stdout  # host setup ran
    assert "ecm2_linear_form_create" in r.stderr and "no HIP device" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), ("3", "1"), ("2", "3")])
def test_rf_example_on_gpu(args):
    if not os.access(BINARY, os.X_OK):
        _build()
    r = subprocess.run([BINARY, *args], cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("PASS")
    assert "converged 1" in r.stdout
