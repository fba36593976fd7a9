"""examples/lesion.cpp: a native caller of the cell-death state through include/ecm2_pa.h alone -- (a) a frozen
slab T(x) = 37 + 58 x: 60 steps of 1 s against one step of 60 s and against the closed form in long double per
dof, and the lesion volume at theta = 0.8 from ecm2_celldeath_measure against the host's sum; (b) ten sourced
SDIRK33 steps each followed by ecm2_celldeath_step(T0 = u_old, T1 = u_new, nsub = 4), with D non-decreasing, all
fractions in [0, 1] and |N + U + D - 1| <= 1e-12 at every step."""
import os
import subprocess

import pytest

from helpers import ROOT

EXAMPLES = os.path.join(ROOT, "examples")
BINARY = os.path.join(EXAMPLES, "lesion")


def _build():
    subprocess.run(["make", "-s", "-C", EXAMPLES], check=True, timeout=300)
    assert os.access(BINARY, os.X_OK)


def test_lesion_example_builds_and_fails_loudly_without_gpu():
    """Compiles and links against the header + library; with no device ecm2_celldeath_create returns
    ECM2_ERR_HIP and the program stops with status 2 (no CPU fallback), after the host setup.  (Where a device is
    visible the run itself is test_lesion_example_on_gpu's.)"""
    _build()
    import ecm2_amd as E
    if E.load_library().ecm2_device_count() > 0:
        return
    r = subprocess.run([BINARY], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "slab 8 x 4 x 4 elements" in r.stdout and "three-state cell death" in r.stdout  # host setup ran
    assert "ecm2_celldeath_create" in r.stderr and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_lesion_example_on_gpu():
    if not os.access(BINARY, os.X_OK):
        _build()
    r = subprocess.run([BINARY], cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("PASS")
    assert "(b) step 10" in r.stdout and "FAILED" not in r.stdout
