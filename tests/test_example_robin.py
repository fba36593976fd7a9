"""examples/robin_heat.cpp: a native caller of the boundary integrators through include/ecm2_pa.h
alone -- a slab with a Dirichlet face, a Robin face (boundary MassIntegrator + BoundaryLFIntegrator on
attribute 3) and insulated sides, solved by constrained Jacobi-PCG and checked against its closed form
u = T0 - h (T0 - T_b) x / (k + h L) (1e-9 relative in the max norm) and sum b = h T_b."""
import os
import subprocess

import pytest

from helpers import ROOT

EXAMPLES = os.path.join(ROOT, "examples")
BINARY = os.path.join(EXAMPLES, "robin_heat")


def _build():
    subprocess.run(["make", "-s", "-C", EXAMPLES], check=True, timeout=300)
    assert os.access(BINARY, os.X_OK)


def test_robin_example_builds_and_fails_loudly_without_gpu():
    """Compiles and links against the header + library; with no device the form's create returns
    ECM2_ERR_HIP and the program stops with status 2 (no CPU fallback).  (Where a device is visible
    the run itself is test_robin_example_on_gpu's.)"""
    _build()
    import ecm2_amd as E
    if E.load_library().ecm2_device_count() > 0:
        return
    r = subprocess.run([BINARY], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "slab 8 x 4 x 4 elements" in r.stdout and "16 Robin" in r.stdout  # host setup ran
    assert "ecm2_pa_form_create" in r.stderr and "no HIP device" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), ("3", "1"), ("2", "3"), ("2", "4", "3")])
def test_robin_example_on_gpu(args):
    if not os.access(BINARY, os.X_OK):
        _build()
    r = subprocess.run([BINARY, *args], cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("PASS")
    assert "converged 1" in r.stdout
